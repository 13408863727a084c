// launch_plan.h -- how the host loops of the iterative solvers batch their launches, and which launches of a batch a profile samples.
//
// Every solver keeps its scalars on the device: the host enqueues a batch of iterations, reads the control block back (one poll) and enqueues the
// next batch.  This header is the one statement of the batch sequence, of the poll count it costs and of the sampling rule; cg_host.h runs a plan.
// Host arithmetic only, no HIP: tests/cpu/launch_plan_check.cpp compiles it alone.
#pragma once

struct LaunchPlan {
    static constexpr int BATCH_CAP = 64;        // doubling stops here; the profile samples inside the first BATCH_CAP launches of a batch
    static constexpr int SAMPLE_STRIDE = 8;     // one launch in eight of those is sampled ...
    static constexpr int SAMPLE_SLOTS = BATCH_CAP / SAMPLE_STRIDE;   // ... into one of eight event slots
    static constexpr int ITER_LIMIT = 200000;   // a loop that gets here has not converged (recorded as a failure)

    int first;          // iterations of the first batch
    int later;          // > 0: of every later batch; 0: each later batch doubles the one before it, up to BATCH_CAP
    int next(int batch) const { return later > 0 ? later : (batch < BATCH_CAP ? batch * 2 : batch); }

    // no hint: `first`, then doubling (K-CG, split-matrix CG and the local-heat CSR solves from 8)
    static LaunchPlan doubling(int first) { return {first, 0}; }
    // The iteration count of consecutive solves of the same system changes slowly (X: 666 +- 10 at 85 k sites), so the first batch is sized just below
    // the previous count; after it, short batches keep the no-op tail small.  (single-vector CG on X, CSR or tiled)
    static LaunchPlan hinted_minus8(int hint) { return hint > 24 ? LaunchPlan{hint - 8, 8} : doubling(8); }
    // The first batch covers three quarters of the previous solve's sweeps -- with the warm start the count moves by +-30 per cent from step to step
    // (9.4e5 sites: 268 ... 505), and a batch sized to the previous count left up to a quarter of its launches as no-ops --, then batches of 8; without
    // a hint batches of 4, 8, ... 64.  (block-CG)
    static LaunchPlan hinted_three_quarters(int hint)
    {
        const int q = hint * 3 / 4;
        return hint > 12 ? LaunchPlan{q > 4 ? q : 4, 8} : doubling(4);
    }

    // read-backs a solve that stops after `iters` iterations costs: one before each batch and the one that sees the stop word
    int polls(int iters) const
    {
        int n = 1, launched = 0;
        for (int batch = first; launched < iters; batch = next(batch)) { launched += batch; ++n; }
        return n;
    }

    // position b of a batch carries events
    static bool sampled(int b) { return b < BATCH_CAP && b % SAMPLE_STRIDE == 0; }
    static int slot(int b) { return b / SAMPLE_STRIDE; }
    // Slots 0 ... n - 1 of a batch of `launched` iterations that began at iteration `start` count in a solve that stopped after `iters`: only
    // launches that did work (iteration index below the final count) are counted.
    static int counted_slots(int start, int launched, int iters)
    {
        int n = 0;
        while (n < SAMPLE_SLOTS && n * SAMPLE_STRIDE < launched && start + n * SAMPLE_STRIDE < iters) ++n;
        return n;
    }
};
